"""CPU: cross pseudo supervision is wired in -- header, binding and library agree on the C ABI (>= 35) and export the two entry
points, whose argument checks answer with an error code before any device call; the oracle's loss with every pixel kept is
the sum of two plain cross-entropies; the hook owns a peer that differs from the model, is reproducible from ``peer_seed``
and travels in ``state_dict``; it refuses what it cannot run; ``create_hook_from_config`` builds it from
``CrossPseudoParameters`` (refused during pre-training, nothing extra without the section)."""
import ctypes
import os
import re

import pytest
import torch

from tests import _cps_oracle as CO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _config(**sections):
    return dict({"Data": {"name": "acdc"}, "Trainer": {"max_epoch": 30}}, **sections)


def _model(seed=0):
    from spcl_amd.semi_seg.arch import UNet
    torch.manual_seed(seed)
    return UNet(input_dim=1, num_classes=4, max_channel=128)


def test_header_binding_and_library_agree_and_export_the_entry_points():
    from spcl_amd import native
    header = open(os.path.join(ROOT, "include", "spcl_hip.h")).read()
    version = int(re.search(r"#define SPCL_ABI_VERSION (\d+)", header).group(1))
    L = native.lib()
    assert version == native.ABI_VERSION == L.spcl_abi_version() and version >= 35
    for name in ("spcl_cross_pseudo_workspace_bytes", "spcl_cross_pseudo_ce"):
        assert name in native._SIGNATURES and name in header
        assert getattr(L, name, None) is not None, name
    res, args = native._SIGNATURES["spcl_cross_pseudo_ce"]
    assert res is ctypes.c_int and len(args) == 18
    assert args[2:6] == [ctypes.c_int] * 4 and args[7] is ctypes.c_float and args[16] is ctypes.c_size_t


def test_workspace_grows_with_the_pixels_and_refuses_what_the_entry_refuses():
    from spcl_amd import native
    ws = native.lib().spcl_cross_pseudo_workspace_bytes
    assert 0 < ws(1, 4, 8, 8) < ws(2, 4, 192, 200) < ws(10, 4, 224, 224)
    assert ws(10, 2, 224, 224) < ws(10, 4, 224, 224) < ws(10, 16, 224, 224)
    # one row of 2 doubles and 4 C + 1 counters per 1024 pixels, and the ticket
    nblk = (10 * 224 * 224 + 1023) // 1024
    assert ws(10, 4, 224, 224) >= nblk * (2 * 8 + 17 * 4) + 4
    assert ws(1, 17, 8, 8) == 0 and ws(1, 0, 8, 8) == 0 and ws(0, 4, 8, 8) == 0 and ws(1, 4, 0, 8) == 0 and ws(1, 4, 8, -1) == 0
    assert ws(32768, 4, 256, 256) == 0  # N H W == 2^31
    assert ws(32767, 4, 256, 256) > 0


def test_argument_checks_report():
    """every refusal below happens on the host, before any device call: an error code and a message, not a crash"""
    from spcl_amd import native
    L = native.lib()
    fake, other = ctypes.c_void_p(4096), ctypes.c_void_p(8192)  # never dereferenced: each call is refused before a launch

    def call(C=4, a=fake, b=fake, loss=fake, parts=fake, da=fake, db=other, hist=fake, ws=fake, ws_bytes=1 << 20, N=3):
        return L.spcl_cross_pseudo_ce(a, b, N, C, 20, 24, None, ctypes.c_float(1.0), loss, parts, da, db, hist, None, None,
                                      ws, ws_bytes, None)

    for kwargs, word in (({"C": 17}, b"C <= 16"), ({"C": 0}, b"C <= 16"), ({"N": 0}, b"bad shape"), ({"a": None}, b"null"),
                         ({"b": None}, b"null"), ({"loss": None}, b"null"), ({"parts": None}, b"null"), ({"da": None}, b"null"),
                         ({"db": None}, b"null"), ({"hist": None}, b"null"), ({"ws": None}, b"null"),
                         ({"ws_bytes": 64}, b"workspace"), ({"db": fake}, b"one buffer"),
                         ({"ws": ctypes.c_void_p(4100)}, b"aligned")):
        assert call(**kwargs) == -1, kwargs
        assert word in L.spcl_last_error(), (kwargs, L.spcl_last_error())


def test_functional_has_no_cpu_path():
    from spcl_amd import functional as F_hip
    t = torch.zeros(1, 4, 8, 8)
    with pytest.raises(RuntimeError, match="MI355X"):
        F_hip.cross_pseudo_ce(t, t)


@pytest.mark.parametrize("weight", [1.0, 2.5])
def test_oracle_with_every_pixel_kept_is_two_plain_cross_entropies(weight):
    g = torch.Generator().manual_seed(23)
    a, b = 3.0 * torch.randn(2, 3, 5, 7, generator=g), 3.0 * torch.randn(2, 3, 5, 7, generator=g)
    (confA, yA), (confB, yB) = CO.conf_and_label(a), CO.conf_and_label(b)
    assert confA.dtype == torch.float64 and torch.equal(yA, a.argmax(1)) and torch.equal(yB, b.argmax(1))
    every = torch.ones_like(yA, dtype=torch.bool)
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    got = CO.loss(a64, b64, yA, yB, every, every, weight)
    ce = torch.nn.functional.cross_entropy
    want = weight * (ce(a.double(), yB) + ce(b.double(), yA))
    assert float(got.detach()) == pytest.approx(float(want), rel=1e-14)
    got.backward()
    assert a64.grad is not None and b64.grad is not None and bool(a64.grad.any()) and bool(b64.grad.any())
    h = CO.hist(yA, yB, every, every, 3)
    assert h.shape == (13,) and int(h[:3].sum()) == int(h[6:9].sum()) == 70 and int(h[12]) == int((yA == yB).sum())
    none = ~every
    assert float(CO.loss(a.double(), b.double(), yA, yB, none, none)) == 0.0
    # the lowest class on a tie, whatever torch.argmax does
    tie = torch.tensor([1.0, 2.0, 2.0]).view(1, 3, 1, 1)
    assert CO.conf_and_label(tie)[1].item() == 1


def test_config_section_builds_the_hook():
    from spcl_amd.hook_creator import create_hook_from_config
    from spcl_amd.semi_seg.hooks import CrossPseudoTrainerHook, create_cross_pseudo_hook
    model = _model()
    params = {"weight": 1.5, "threshold": 0.8, "peer_seed": 3, "on": ["unlabeled", "unlabeled_tf"]}
    (hook,) = create_hook_from_config(model, _config(CrossPseudoParameters=params))
    assert isinstance(hook, CrossPseudoTrainerHook) and hook._hook_name == "cps" and hook._weight == 1.5
    assert hook._on == ("unlabeled", "unlabeled_tf") and hook._peer_seed == 3
    assert hook.tau.dtype == torch.float32 and hook.tau.tolist() == pytest.approx([0.8] * 4)
    assert hook.thresholds(torch.device("cpu")) is hook.tau
    with pytest.raises(RuntimeError):
        create_hook_from_config(model, _config(CrossPseudoParameters=params), is_pretrain=True)
    assert create_hook_from_config(model, _config()) == []  # configs without the section behave as before
    plain = create_cross_pseudo_hook(model=model, weight=2.0)
    assert plain.tau.tolist() == [0.0] * 4 and plain.thresholds(torch.device("cpu")) is None  # plain CPS passes no vector
    assert plain._on == ("labeled", "unlabeled", "unlabeled_tf")
    assert plain().graph_key() == ("_CrossPseudoEpocherHook", 2.0, ("labeled", "unlabeled", "unlabeled_tf"), "plain")
    assert hook().graph_key() == ("_CrossPseudoEpocherHook", 1.5, ("unlabeled", "unlabeled_tf"), "tau")


def test_the_peer_is_learnable_differs_from_the_model_and_follows_its_seed():
    from spcl_amd.semi_seg.hooks import CrossPseudoTrainerHook
    model = _model()
    before = [p.detach().clone() for p in model.parameters()]
    rng = torch.random.get_rng_state()
    hook = CrossPseudoTrainerHook("cps", 1.0, model)
    assert torch.equal(torch.random.get_rng_state(), rng)  # the peer is drawn inside a seeded context that is put back
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), before))
    peer = hook.peer
    assert hook.learnable_modules == [peer] and peer is not model and type(peer) is type(model)
    assert (peer._input_dim, peer.num_classes, peer._max_channel) == (model._input_dim, model.num_classes, model._max_channel)
    mine, theirs = list(hook.parameters()), list(peer.parameters())
    assert len(mine) == len(theirs) == len(before) and all(p is q for p, q in zip(mine, theirs))
    assert all(p.requires_grad for p in mine)
    assert [p.shape for p in theirs] == [p.shape for p in before]
    assert any(not torch.equal(p, q) for p, q in zip(theirs, before))
    assert isinstance(CrossPseudoTrainerHook.peer, property) and CrossPseudoTrainerHook.peer.fset is None  # read only
    # the same seed, the same peer; another seed, another peer -- whatever the global generator holds
    torch.manual_seed(12345)
    again = CrossPseudoTrainerHook("cps", 1.0, model)
    assert all(torch.equal(p, q) for p, q in zip(again.peer.parameters(), theirs))
    other = CrossPseudoTrainerHook("cps", 1.0, model, peer_seed=2)
    assert any(not torch.equal(p, q) for p, q in zip(other.peer.parameters(), theirs))
    # a given peer is taken as it is
    given = _model(seed=7)
    assert CrossPseudoTrainerHook("cps", 1.0, model, peer=given).peer is given


def test_batchnorm_momentum_of_the_model_reaches_the_peer():
    from spcl_amd.semi_seg.arch import UNet
    from spcl_amd.semi_seg.hooks import CrossPseudoTrainerHook
    model = UNet(input_dim=1, num_classes=4, max_channel=128, momentum=0.03)
    peer = CrossPseudoTrainerHook("cps", 1.0, model).peer
    moms = {m.momentum for m in peer.modules() if isinstance(m, torch.nn.BatchNorm2d)}
    assert moms == {0.03}


def test_the_hook_refuses_what_it_cannot_run():
    from copy import deepcopy
    from spcl_amd.semi_seg.hooks import CrossPseudoTrainerHook
    model = _model()
    with pytest.raises(ValueError, match="identical"):
        CrossPseudoTrainerHook("cps", 1.0, model, peer=deepcopy(model))
    with pytest.raises(ValueError, match="identical"):
        CrossPseudoTrainerHook("cps", 1.0, model, peer=model)
    for bad in (1.5, -0.1, [0.5, 0.5, 0.5, 1.01], [0.5, -1e-3, 0.5, 0.5]):
        with pytest.raises(ValueError, match="threshold"):
            CrossPseudoTrainerHook("cps", 1.0, model, threshold=bad)
    with pytest.raises(ValueError, match="thresholds for 4 classes"):
        CrossPseudoTrainerHook("cps", 1.0, model, threshold=[0.5, 0.6, 0.7])
    with pytest.raises(ValueError, match="thresholds for 4 classes"):
        CrossPseudoTrainerHook("cps", 1.0, model, threshold=[0.5] * 5)
    with pytest.raises(ValueError, match="empty"):
        CrossPseudoTrainerHook("cps", 1.0, model, on=())
    with pytest.raises(ValueError, match="none of"):
        CrossPseudoTrainerHook("cps", 1.0, model, on=("labeled", "unlabelled"))
    for good in (0.0, 1.0, [0.0, 0.25, 0.5, 1.0]):
        CrossPseudoTrainerHook("cps", 1.0, model, threshold=good)


def test_the_state_dict_holds_the_peer_and_the_thresholds():
    from spcl_amd.semi_seg.hooks import CrossPseudoTrainerHook
    model = _model()
    hook = CrossPseudoTrainerHook("cps", 1.0, model, threshold=[0.5, 0.6, 0.7, 0.8])
    sd = hook.state_dict()
    assert "tau" in sd and sd["tau"].tolist() == pytest.approx([0.5, 0.6, 0.7, 0.8])
    assert sorted(k for k in sd if k != "tau") == sorted("_peer." + k for k in model.state_dict())
    # a hook with another peer takes the saved one over, bit for bit (running statistics included)
    late = CrossPseudoTrainerHook("cps", 1.0, model, peer_seed=9)
    assert any(not torch.equal(p, q) for p, q in zip(late.peer.parameters(), hook.peer.parameters()))
    late.load_state_dict(sd)
    for k, v in hook.peer.state_dict().items():
        assert torch.equal(late.peer.state_dict()[k], v), k
    assert torch.equal(late.tau, hook.tau)


def test_a_call_without_the_images_says_so():
    """an epocher with another keyword set (MixUpEpocher hands over ``labeled_image`` / ``labeled_image_tf``) never gives the
    hook the three batches: a RuntimeError that names the cause, before any device work"""
    from spcl_amd.semi_seg.hooks import CrossPseudoTrainerHook

    from contextlib import nullcontext

    class _Meters(dict):
        def register_meter(self, key, meter):
            self[key] = meter

        def focus_on(self, name):
            return nullcontext()

    class MixUpEpocher:
        meters = _Meters()

    epocher = MixUpEpocher()
    hook = CrossPseudoTrainerHook("cps", 1.0, _model())()
    hook.set_epocher(epocher)
    assert sorted(epocher.meters) == ["agree", "kept", "loss", "peer_sup_loss"]
    x = torch.zeros(1, 1, 8, 8)
    logits = torch.zeros(1, 4, 8, 8)
    hook.before_forward_pass(labeled_image=x, labeled_image_tf=x)
    assert hook._images is None
    target = torch.zeros(1, 1, 8, 8, dtype=torch.long)
    with pytest.raises(RuntimeError, match="MixUpEpocher.*image batches"):  # the keywords of MixUpEpocher.step, no others
        hook(labeled_image=x, labeled_image_tf=x, labeled_target=target, labeled_target_tf=target, seed=1, label_logits=logits)
    hook.before_forward_pass(labeled_image=x, unlabeled_image=x, unlabeled_image_tf=x)
    with pytest.raises(RuntimeError, match="image batches"):  # the images alone do not do: the three class maps are missing
        hook(labeled_target=target, label_logits=logits)
    assert hook._images is None
    hook.before_forward_pass(labeled_image=x, unlabeled_image=x, unlabeled_image_tf=x)
    assert all(t is x for t in hook._images)  # references, no copies
