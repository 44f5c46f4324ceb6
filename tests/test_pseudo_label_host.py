"""CPU: the pseudo-labelling baseline is wired in -- header, binding and library agree on the C ABI and export the two entry
points, whose argument checks answer with an error code before any device call; ``functional.pseudo_label_ce`` has no CPU
path; the hook refuses what it cannot run; the factory and ``create_hook_from_config`` build it from
``PseudoLabelParameters`` (refused during pre-training, nothing extra without the section); the oracle's ``update()``
reproduces a three-class example worked by hand."""
import ctypes
import os
import re

import pytest
import torch

from tests import _pseudo_label_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _config(**sections):
    return dict({"Data": {"name": "acdc"}, "Trainer": {"max_epoch": 30}}, **sections)


def _model():
    from spcl_amd.semi_seg.arch import UNet
    return UNet(input_dim=1, num_classes=4, max_channel=128)


def test_header_binding_and_library_agree_and_export_the_entry_points():
    from spcl_amd import native
    header = open(os.path.join(ROOT, "include", "spcl_hip.h")).read()
    version = int(re.search(r"#define SPCL_ABI_VERSION (\d+)", header).group(1))
    L = native.lib()
    assert version == native.ABI_VERSION == L.spcl_abi_version() and version >= 33
    for name in ("spcl_pseudo_label_workspace_bytes", "spcl_pseudo_label_ce"):
        assert name in native._SIGNATURES and name in header
        assert getattr(L, name, None) is not None, name


def test_workspace_grows_with_the_pixels_and_with_the_classes():
    from spcl_amd import native
    ws = native.lib().spcl_pseudo_label_workspace_bytes
    assert 0 < ws(1, 4, 8, 8) < ws(2, 4, 192, 200) < ws(10, 4, 224, 224)
    assert ws(10, 2, 224, 224) < ws(10, 4, 224, 224) < ws(10, 16, 224, 224)
    # one row of 2 + C doubles and 2 C counters per 1024 pixels, and the ticket
    nblk = (10 * 224 * 224 + 1023) // 1024
    assert ws(10, 4, 224, 224) >= nblk * (6 * 8 + 8 * 4) + 4
    assert ws(1, 17, 8, 8) == 0 and ws(0, 4, 8, 8) == 0


def test_argument_checks_report():
    """every refusal below happens on the host, before any device call: an error code and a message, not a crash"""
    from spcl_amd import native
    L = native.lib()
    fake = ctypes.c_void_p(4096)  # never dereferenced: each call below is refused before a launch

    def call(C=4, teacher=fake, student=fake, tau=fake, state=None, momentum=0.999, loss=fake, ds=fake, stats=fake, hist=fake,
             ws=fake, ws_bytes=1 << 20, N=3):
        return L.spcl_pseudo_label_ce(teacher, student, N, C, 20, 24, None, tau, state, ctypes.c_double(momentum),
                                      ctypes.c_float(1.0), loss, ds, stats, hist, None, ws, ws_bytes, None)

    for kwargs, word in (({"C": 17}, b"C <= 16"), ({"C": 0}, b"C <= 16"), ({"N": 0}, b"bad shape"),
                         ({"teacher": None}, b"null"), ({"student": None}, b"null"), ({"tau": None}, b"null"),
                         ({"loss": None}, b"null"), ({"ds": None}, b"null"), ({"stats": None}, b"null"),
                         ({"hist": None}, b"null"), ({"ws": None}, b"null"), ({"ws_bytes": 64}, b"workspace"),
                         ({"state": fake, "momentum": 1.0}, b"momentum"), ({"state": fake, "momentum": -0.1}, b"momentum")):
        assert call(**kwargs) == -1, kwargs
        assert word in L.spcl_last_error(), (kwargs, L.spcl_last_error())


def test_functional_has_no_cpu_path():
    from spcl_amd import functional as F_hip
    t = torch.zeros(1, 4, 8, 8)
    with pytest.raises(RuntimeError, match="MI355X"):
        F_hip.pseudo_label_ce(t, t, torch.full((4,), 0.5))
    with pytest.raises(ValueError, match="momentum"):
        F_hip.pseudo_label_ce(t, t, torch.full((4,), 0.5), momentum=1.0)
    tau, state = F_hip.pseudo_label_state(3, "cpu")
    assert tau.dtype == torch.float32 and tau.tolist() == [pytest.approx(1 / 3)] * 3
    assert state.dtype == torch.float64 and state.shape == (4,) and float(state[0]) == 1.0 / 3.0
    with pytest.raises(ValueError):
        F_hip.pseudo_label_state(17, "cpu")


def test_the_hook_refuses_what_it_cannot_run():
    from spcl_amd.semi_seg.hooks import PseudoLabelTrainerHook
    model = _model()
    with pytest.raises(ValueError, match="teacher"):
        PseudoLabelTrainerHook("pseudolabel", 1.0, model, teacher="student")
    with pytest.raises(ValueError, match="ema"):
        PseudoLabelTrainerHook("pseudolabel", 1.0, teacher="ema")
    for bad in (0.0, 1.5, -0.1, [0.5, 0.5, 0.5, 1.01]):
        with pytest.raises(ValueError, match="threshold"):
            PseudoLabelTrainerHook("pseudolabel", 1.0, model, threshold=bad)
    with pytest.raises(ValueError, match="thresholds for 4 classes"):
        PseudoLabelTrainerHook("pseudolabel", 1.0, model, threshold=[0.5, 0.6, 0.7])
    with pytest.raises(ValueError, match="thresholds for 4 classes"):  # ignored in value, not in length
        PseudoLabelTrainerHook("pseudolabel", 1.0, model, threshold=[0.5, 0.6, 0.7], adaptive=True)
    with pytest.raises(ValueError, match="momentum"):
        PseudoLabelTrainerHook("pseudolabel", 1.0, model, adaptive=True, momentum=1.0)


def test_the_hook_owns_its_thresholds_as_buffers():
    from spcl_amd.semi_seg.hooks import MeanTeacherTrainerHook, PseudoLabelTrainerHook
    model = _model()
    fixed = PseudoLabelTrainerHook("pseudolabel", 1.0, model, threshold=[0.5, 0.6, 0.7, 0.8])
    assert sorted(fixed.state_dict()) == ["tau"] and fixed.tau.tolist() == pytest.approx([0.5, 0.6, 0.7, 0.8])
    assert fixed.teacher_model is None and list(fixed.parameters()) == []
    assert fixed().graph_key() == ("_PseudoLabelEpocherHook", 1.0, 0.999, "fixed")
    adaptive = PseudoLabelTrainerHook("pseudolabel", 1.0, model, adaptive=True, momentum=0.9)
    assert sorted(adaptive.state_dict()) == ["state", "tau"]
    assert adaptive.tau.tolist() == [0.25] * 4 and adaptive.state.tolist() == [0.25] * 5
    assert adaptive().graph_key() == ("_PseudoLabelEpocherHook", 1.0, 0.9, "adaptive")
    ema = PseudoLabelTrainerHook("pseudolabel", 1.0, model, teacher="ema")
    assert isinstance(ema, MeanTeacherTrainerHook) and ema.teacher_model is not model
    assert all(not p.requires_grad for p in ema.teacher_model.parameters())
    assert ema().graph_key() is None  # (the moving average's alpha_t changes with every step)
    # no model: built by the first call -- or by a checkpoint that is loaded before it
    adaptive.state.copy_(torch.tensor([0.7, 0.1, 0.2, 0.3, 0.4], dtype=torch.float64))
    adaptive.tau.copy_(torch.tensor([0.2, 0.3, 0.5, 0.7]))
    late = PseudoLabelTrainerHook("pseudolabel", 1.0, adaptive=True, momentum=0.9)
    assert late.tau is None and late.state_dict() == {}
    late.load_state_dict(adaptive.state_dict())
    assert torch.equal(late.tau, adaptive.tau) and torch.equal(late.state, adaptive.state)
    assert late.state.dtype == torch.float64
    with pytest.raises(ValueError, match="class maps of 3"):
        late.thresholds(3, torch.device("cpu"))


def test_config_section_builds_the_hook():
    from spcl_amd.hook_creator import create_hook_from_config
    from spcl_amd.semi_seg.hooks import PseudoLabelTrainerHook, create_pseudo_label_hook
    model = _model()
    params = {"weight": 0.5, "threshold": 0.9, "adaptive": True, "momentum": 0.99}
    (hook,) = create_hook_from_config(model, _config(PseudoLabelParameters=params))
    assert isinstance(hook, PseudoLabelTrainerHook) and hook._hook_name == "pseudolabel" and hook._weight == 0.5
    assert (hook._adaptive, hook._momentum, hook._teacher) == (True, 0.99, "self")
    with pytest.raises(RuntimeError):
        create_hook_from_config(model, _config(PseudoLabelParameters=params), is_pretrain=True)
    assert create_hook_from_config(model, _config()) == []  # configs without the section behave as before
    plain = create_pseudo_label_hook(model=model, weight=2.0)
    assert plain.tau.tolist() == pytest.approx([0.95] * 4) and plain.state is None


def test_update_reproduces_a_hand_worked_example():
    """three classes, 10 pixels, momentum 0.5, state (0.5; 0.2, 0.3, 0.5), stats (8; 5, 3, 2):
    tau_g' = 0.5 * 0.5 + 0.5 * 0.8 = 0.65;  ptilde' = (0.1 + 0.25, 0.15 + 0.15, 0.25 + 0.1) = (0.35, 0.3, 0.35);
    tau' = ptilde' / 0.35 * 0.65 = (0.65, 0.3 / 0.35 * 0.65 = 0.557142857..., 0.65)"""
    state = torch.tensor([0.5, 0.2, 0.3, 0.5], dtype=torch.float64)
    stats = torch.tensor([8.0, 5.0, 3.0, 2.0], dtype=torch.float64)
    new, tau = PO.update(state, stats, 10, 0.5)
    assert new.tolist() == pytest.approx([0.65, 0.35, 0.3, 0.35], rel=1e-15)
    assert tau.tolist() == pytest.approx([0.65, 0.39 / 0.7, 0.65], rel=1e-15)
    # momentum 0 forgets the past: the state is the batch's means
    new, tau = PO.update(state, stats, 10, 0.0)
    assert new.tolist() == pytest.approx([0.8, 0.5, 0.3, 0.2], rel=1e-15)
    assert tau.tolist() == pytest.approx([0.8, 0.48, 0.32], rel=1e-15)
